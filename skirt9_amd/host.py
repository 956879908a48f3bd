"""ctypes binding of the host model layer (libskirthost.so, include/skirt_host.h).

The host layer reads an unchanged SKIRT ``.ski`` file, runs the reference's setup for the supported classes and
exposes the flattened ``pmc_scene`` that the HIP engine (``skirt9_amd.engine``) consumes; after the photon loop it
calibrates the detector arrays and writes SKIRT's output files.  Mirrors the call sequence of
``SkirtCommandLineHandler::doSimulation`` (SKIRT/main/SkirtCommandLineHandler.cpp:295-372):
``load -> setup -> [engine] -> write``.
"""
import ctypes as C
import os

_LIBDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")


class FrameLayout(C.Structure):
    """pmc_frame_layout (include/pmc.h)"""
    _fields_ = [("num_components", C.c_int64), ("npix", C.c_int64), ("num_lambda", C.c_int64),
                ("sed_offset", C.c_int64), ("ifu_offset", C.c_int64), ("wsed_offset", C.c_int64),
                ("wifu_offset", C.c_int64), ("end_offset", C.c_int64)]


class CounterValues(C.Structure):
    """pmc_counter_values (include/pmc.h)"""
    _fields_ = [("histories", C.c_uint64), ("paths", C.c_uint64), ("cell_visits", C.c_uint64),
                ("detector_updates", C.c_uint64), ("scatterings", C.c_uint64), ("stat_overflows", C.c_uint64),
                ("rewalk_visits", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


_lib = None


class ScenePointer(int):
    """address of a pmc_scene; ``ext`` is the address of the pmc_scene_ext that belongs to it (the phase function of every medium
    component, the velocity of every source), which ``skirt9_amd.engine.Engine`` hands to pmc_create_ext.  A plain int in its place means: no extension."""
    ext = None

    def __new__(cls, scene, ext):
        self = super().__new__(cls, scene)
        self.ext = ext
        return self


# ---- ctypes mirrors of the leading members of pmc_scene (include/pmc.h): inspection of the tables a Simulation hands over

class Grid(C.Structure):
    _fields_ = [("kind", C.c_int32), ("xmin", C.c_double), ("ymin", C.c_double), ("zmin", C.c_double),
                ("xmax", C.c_double), ("ymax", C.c_double), ("zmax", C.c_double), ("eps", C.c_double),
                ("num_cells", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("xv", C.POINTER(C.c_double)), ("yv", C.POINTER(C.c_double)), ("zv", C.POINTER(C.c_double)),
                ("num_nodes", C.c_int32), ("node_box", C.POINTER(C.c_double)), ("node_level", C.POINTER(C.c_int32)),
                ("node_first_child", C.POINTER(C.c_int32)), ("node_cell", C.POINTER(C.c_int32)),
                ("nbr_start", C.POINTER(C.c_int32)), ("nbr_list", C.POINTER(C.c_int32)),
                ("site", C.POINTER(C.c_double)), ("vnbr_start", C.POINTER(C.c_int32)), ("vnbr_list", C.POINTER(C.c_int32)),
                ("vblock_n", C.c_int32), ("vblock_start", C.POINTER(C.c_int32)), ("vblock_list", C.POINTER(C.c_int32))]


class Medium(C.Structure):
    _fields_ = [("number_density", C.POINTER(C.c_double)), ("num_lambda", C.c_int32),
                ("lambda_border", C.POINTER(C.c_double)), ("sigma_ext", C.POINTER(C.c_double)),
                ("sigma_sca", C.POINTER(C.c_double)), ("asymmpar", C.POINTER(C.c_double)),
                ("sigma_abs", C.POINTER(C.c_double))]


class SourceVelocity(C.Structure):
    """pmc_source_velocity (include/pmc.h): kind = PMC_VELOCITY_* (0 at rest, 1 constant, 2 radial, 3 cylindrical)"""
    _fields_ = [("kind", C.c_int32), ("magnitude", C.c_double), ("vector", C.c_double * 3), ("unity_radius", C.c_double),
                ("exponent", C.c_double)]

    def as_dict(self):
        return {"kind": int(self.kind), "magnitude": float(self.magnitude), "vector": tuple(self.vector),
                "unity_radius": float(self.unity_radius), "exponent": float(self.exponent)}


class SceneExt(C.Structure):
    """pmc_scene_ext (include/pmc.h)"""
    _fields_ = [("struct_size", C.c_int32), ("phase_function", C.c_int32 * 4), ("source_velocity", SourceVelocity * 16)]


class SceneHead(C.Structure):
    """leading members of pmc_scene (include/pmc.h)"""
    _fields_ = [("abi_version", C.c_int32), ("grid", Grid), ("medium", Medium)]


class ProbeMapInfo(C.Structure):
    """skh_probe_map (include/skirt_host.h)"""
    _fields_ = [("file_name", C.c_char * 256), ("nx", C.c_int32), ("ny", C.c_int32), ("sampling", C.c_int32), ("num_values", C.c_int32),
                ("after_setup", C.c_int32), ("num_rays", C.c_int64)]


# skh_integrate_fn (include/skirt_host.h)
INTEGRATE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double),
                           C.POINTER(C.c_double))


# skh_integrate_weighted_fn and skh_temperature_fn (include/skirt_host.h)
INTEGRATE_WEIGHTED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double))
TEMPERATURE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double))


# skh_sample_fn (include/skirt_host.h)
SAMPLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                        C.POINTER(C.c_int32))


class DustHeating(C.Structure):
    """pmc_dust_heating (include/pmc.h)"""
    _fields_ = [("num_components", C.c_int32), ("num_lambda", C.c_int32), ("num_temperatures", C.c_int32), ("num_cells", C.c_int32),
                ("width", C.POINTER(C.c_double)), ("sigma", C.POINTER(C.c_double)), ("planckabs", C.POINTER(C.c_double)),
                ("temperature", C.POINTER(C.c_double)), ("cell_factor", C.POINTER(C.c_double)), ("mass_density", C.POINTER(C.c_double))]


class AdaptiveMesh(C.Structure):
    """pmc_adaptive_mesh (include/pmc.h)"""
    _fields_ = [("num_nodes", C.c_int32), ("num_cells", C.c_int32), ("node_box", C.POINTER(C.c_double)), ("node_dims", C.POINTER(C.c_int32)),
                ("node_link", C.POINTER(C.c_int32)), ("cell_density", C.POINTER(C.c_double))]


MESH_ARRAYS = ("node_box", "node_dims", "node_link", "cell_density")


def mesh_struct(tables):
    """the pmc_adaptive_mesh of a dict as ``Simulation.adaptive_mesh`` returns it (sizes from the shapes of the arrays); returns
    (struct, arrays): the struct points into the arrays, which the caller keeps alive while it is in use"""
    import numpy as np
    arrays = {"node_box": np.ascontiguousarray(tables["node_box"], dtype=np.float64).reshape(-1, 6),
              "node_dims": np.ascontiguousarray(tables["node_dims"], dtype=np.int32).reshape(-1, 3),
              "node_link": np.ascontiguousarray(tables["node_link"], dtype=np.int32).reshape(-1),
              "cell_density": np.ascontiguousarray(tables["cell_density"], dtype=np.float64).reshape(-1)}
    n = arrays["node_link"].shape[0]
    if arrays["node_box"].shape[0] != n or arrays["node_dims"].shape[0] != n:
        raise ValueError("node_box, node_dims and node_link must describe the same nodes")
    struct = AdaptiveMesh(n, arrays["cell_density"].shape[0])
    for name in MESH_ARRAYS:
        ctype = C.c_double if arrays[name].dtype == np.float64 else C.c_int32
        setattr(struct, name, arrays[name].ctypes.data_as(C.POINTER(ctype)))
    return struct, arrays


class ProbeEngine(C.Structure):
    """skh_probe_engine (include/skirt_host.h)"""
    _fields_ = [("integrate", C.c_void_p), ("integrate_weighted", C.c_void_p), ("temperatures", C.c_void_p), ("user", C.c_void_p),
                ("rf", C.c_void_p)]


HEATING_ARRAYS = ("width", "sigma", "planckabs", "temperature", "cell_factor", "mass_density")


def heating_tables_from(struct):
    """a pmc_dust_heating as a dict of numpy arrays (copies): width [L], sigma [H][L], planckabs [H][NT], temperature [NT], cell_factor [cells],
    mass_density [H][cells]"""
    import numpy as np
    H, L, NT, cells = struct.num_components, struct.num_lambda, struct.num_temperatures, struct.num_cells
    shapes = {"width": (L,), "sigma": (H, L), "planckabs": (H, NT), "temperature": (NT,), "cell_factor": (cells,), "mass_density": (H, cells)}
    return {name: np.ctypeslib.as_array(getattr(struct, name), shape=shapes[name]).copy() for name in HEATING_ARRAYS}


def heating_struct(tables):
    """the pmc_dust_heating of a dict as ``Simulation.temperature_tables`` returns it (sizes from the shapes of the arrays); returns
    (struct, arrays): the struct points into the arrays, which the caller keeps alive while it is in use"""
    import numpy as np
    arrays = {name: np.ascontiguousarray(tables[name], dtype=np.float64) for name in HEATING_ARRAYS}
    sigma, planck, rho = arrays["sigma"], arrays["planckabs"], arrays["mass_density"]
    if sigma.ndim != 2 or planck.ndim != 2 or rho.ndim != 2 or not (sigma.shape[0] == planck.shape[0] == rho.shape[0]):
        raise ValueError("sigma, planckabs and mass_density must be [H][...] for the same H")
    if (arrays["width"].shape != (sigma.shape[1],) or arrays["temperature"].shape != (planck.shape[1],)
            or arrays["cell_factor"].shape != (rho.shape[1],)):
        raise ValueError("width, temperature and cell_factor do not match sigma, planckabs and mass_density")
    struct = DustHeating(sigma.shape[0], sigma.shape[1], planck.shape[1], rho.shape[1])
    for name in HEATING_ARRAYS:
        setattr(struct, name, arrays[name].ctypes.data_as(C.POINTER(C.c_double)))
    return struct, arrays


def dust_temperatures(tables, rf):
    """the CPU restatement of the engine's dust temperature kernel for any tables (skh_dust_temperatures_from): [H + 1][num_cells] from
    rf[m * L + ell]"""
    import numpy as np
    struct, keep = heating_struct(tables)
    data = np.ascontiguousarray(rf, dtype=np.float64).reshape(-1)
    if data.size != struct.num_cells * struct.num_lambda:
        raise ValueError("the radiation field table does not match the tables")
    out = np.empty((struct.num_components + 1, struct.num_cells), dtype=np.float64)
    if lib().skh_dust_temperatures_from(C.byref(struct), data.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
        raise RuntimeError(lib().skh_last_error().decode())
    del keep
    return out


def scene_head(sim):
    """the leading members (grid, medium) of the pmc_scene of a set-up Simulation, for inspection"""
    return SceneHead.from_address(sim.scene)


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(_LIBDIR, "libskirthost.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make` (or __graft_entry__.build()) first")
        L = C.CDLL(path)
        L.skh_last_error.restype = C.c_char_p
        L.skh_load.restype = C.c_void_p
        L.skh_load.argtypes = [C.c_char_p]
        L.skh_free.argtypes = [C.c_void_p]
        L.skh_set_num_packets.argtypes = [C.c_void_p, C.c_uint64]
        L.skh_set_tree_topology_file.argtypes = [C.c_void_p, C.c_char_p]
        L.skh_setup.argtypes = [C.c_void_p]
        L.skh_scene.restype = C.c_void_p
        L.skh_scene.argtypes = [C.c_void_p]
        L.skh_scene_ext.restype = C.c_void_p
        L.skh_scene_ext.argtypes = [C.c_void_p]
        L.skh_num_packets.restype = C.c_uint64
        L.skh_num_packets.argtypes = [C.c_void_p]
        L.skh_seed.restype = C.c_int32
        L.skh_seed.argtypes = [C.c_void_p]
        L.skh_packet_luminosity.restype = C.c_double
        L.skh_packet_luminosity.argtypes = [C.c_void_p, C.c_int32]
        L.skh_setup_draws.restype = C.c_uint64
        L.skh_setup_draws.argtypes = [C.c_void_p]
        L.skh_frame_size.restype = C.c_int64
        L.skh_frame_size.argtypes = [C.c_void_p]
        L.skh_frame_layout.argtypes = [C.c_void_p, C.c_int32, C.POINTER(FrameLayout)]
        L.skh_write.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
        L.skh_summary.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
        L.skh_set_particle_sampler.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.skh_set_mesh_sampler.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.skh_adaptive_mesh.argtypes = [C.c_void_p, C.c_int32, C.POINTER(AdaptiveMesh)]
        L.skh_imported_mass.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
        L.skh_imported_densities.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
        L.skh_radiation_field_size.restype = C.c_int64
        L.skh_radiation_field_size.argtypes = [C.c_void_p]
        L.skh_write_radiation_field.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
        L.skh_num_probe_maps.restype = C.c_int32
        L.skh_num_probe_maps.argtypes = [C.c_void_p]
        L.skh_probe_map_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ProbeMapInfo)]
        L.skh_probe_map_rays.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.skh_probe_map_values.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.skh_write_probes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
        L.skh_write_probes_when.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int32]
        L.skh_probe_map_averaged.restype = C.c_int32
        L.skh_probe_map_averaged.argtypes = [C.c_void_p, C.c_int32]
        L.skh_probes_need_radiation_field.restype = C.c_int32
        L.skh_probes_need_radiation_field.argtypes = [C.c_void_p, C.c_int32]
        L.skh_write_probes_with.argtypes = [C.c_void_p, C.POINTER(ProbeEngine), C.c_char_p, C.c_int32]
        L.skh_cell_indices.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.skh_write_probes_sampled.argtypes = [C.c_void_p, C.POINTER(ProbeEngine), C.c_void_p, C.c_char_p, C.c_int32]
        L.skh_dimension.restype = C.c_int32
        L.skh_dimension.argtypes = [C.c_void_p]
        L.skh_dust_heating.argtypes = [C.c_void_p, C.POINTER(DustHeating)]
        L.skh_dust_components.restype = C.c_int32
        L.skh_dust_components.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.skh_dust_temperatures.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.skh_dust_temperatures_from.argtypes = [C.POINTER(DustHeating), C.c_void_p, C.c_void_p]
        L.skh_scene_save.argtypes = [C.c_void_p, C.c_char_p]
        L.skh_scene_load.restype = C.c_void_p
        L.skh_scene_load.argtypes = [C.c_char_p]
        L.skh_scene_file_free.argtypes = [C.c_void_p]
        L.skh_scene_file_scene.restype = C.c_void_p
        L.skh_scene_file_scene.argtypes = [C.c_void_p]
        L.skh_scene_file_scene_ext.restype = C.c_void_p
        L.skh_scene_file_scene_ext.argtypes = [C.c_void_p]
        L.skh_scene_file_number.restype = C.c_int64
        L.skh_scene_file_number.argtypes = [C.c_void_p, C.c_int32]
        L.skh_scene_file_layout.argtypes = [C.c_void_p, C.c_int32, C.POINTER(FrameLayout)]
        _lib = L
    return _lib


class Simulation:
    """A MonteCarloSimulation constructed from a ski file."""

    def __init__(self, ski_path, num_packets=None, tree_topology=None):
        L = lib()
        self.path = str(ski_path)
        self._h = L.skh_load(os.fsencode(ski_path))
        if not self._h:
            raise RuntimeError(L.skh_last_error().decode())
        if num_packets is not None:
            L.skh_set_num_packets(self._h, int(num_packets))
        if tree_topology is not None:
            if L.skh_set_tree_topology_file(self._h, os.fsencode(tree_topology)) != 0:
                raise RuntimeError(L.skh_last_error().decode())
        self._setup = False

    def use_device_sampler(self, device=0):
        """before setup(): evaluate the densities of an imported medium -- smoothed particles or the cells of an adaptive mesh -- on the
        MI355X (libpmc.so pmc_sampler_*): bit-identical to the host evaluation, and the setup of 10^6 particles takes seconds"""
        from . import engine
        E = engine.lib()
        ptr = lambda f: C.cast(f, C.c_void_p)  # noqa: E731
        if lib().skh_set_particle_sampler(self._h, ptr(E.pmc_sampler_create), ptr(E.pmc_sampler_density),
                                          ptr(E.pmc_sampler_destroy), ptr(E.pmc_last_error), device) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        if lib().skh_set_mesh_sampler(self._h, ptr(E.pmc_sampler_create_mesh), ptr(E.pmc_sampler_density),
                                      ptr(E.pmc_sampler_destroy), ptr(E.pmc_last_error), device) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        return self

    def setup(self):
        if lib().skh_setup(self._h) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        self._setup = True
        return self

    def close(self):
        if self._h:
            lib().skh_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def scene(self):
        """address of the pmc_scene, with that of its extension (valid while this object lives)"""
        assert self._setup, "call setup() first"
        return ScenePointer(lib().skh_scene(self._h), lib().skh_scene_ext(self._h))

    @property
    def phase_functions(self):
        """PMC_PHASE_* of every medium component slot (pmc_scene_ext::phase_function)"""
        assert self._setup, "call setup() first"
        return list(SceneExt.from_address(lib().skh_scene_ext(self._h)).phase_function)

    @property
    def source_velocities(self):
        """pmc_scene_ext::source_velocity of every source slot, as dicts (kind 0: at rest)"""
        assert self._setup, "call setup() first"
        return [v.as_dict() for v in SceneExt.from_address(lib().skh_scene_ext(self._h)).source_velocity]

    @property
    def num_packets(self):
        return int(lib().skh_num_packets(self._h))

    @property
    def seed(self):
        return int(lib().skh_seed(self._h))

    def packet_luminosity(self, index=0):
        """luminosity carried by one launched packet at oligochromatic wavelength `index`"""
        value = float(lib().skh_packet_luminosity(self._h, index))
        if value < 0:
            raise ValueError("not an oligochromatic simulation, or wavelength index out of range")
        return value

    @property
    def setup_draws(self):
        return int(lib().skh_setup_draws(self._h))

    @property
    def frame_size(self):
        return int(lib().skh_frame_size(self._h))

    def layout(self, instrument=0):
        out = FrameLayout()
        if lib().skh_frame_layout(self._h, instrument, C.byref(out)) != 0:
            raise IndexError(instrument)
        return out

    @property
    def radiation_field_size(self):
        """doubles of the radiation field table rf[m * nbins + ell]; 0 if the simulation does not store it"""
        return int(lib().skh_radiation_field_size(self._h))

    def write_radiation_field(self, rf, outdir):
        """write the RadiationFieldProbe files (<prefix>_<probe>_J.dat) from the table the engine accumulated"""
        import numpy as np
        data = np.ascontiguousarray(rf, dtype=np.float64)
        assert data.size == self.radiation_field_size
        os.makedirs(outdir, exist_ok=True)
        if lib().skh_write_radiation_field(self._h, data.ctypes.data_as(C.c_void_p), os.fsencode(outdir)) != 0:
            raise RuntimeError(lib().skh_last_error().decode())

    def probe_maps(self):
        """the projected maps (DensityProbe / OpacityProbe / TemperatureProbe with a ParallelProjectionForm) in file order, one dict each:
        file_name, nx, ny, sampling, num_values, num_rays, after_setup, averaged, and the arrays origins [num_rays][3], directions
        [num_rays][3] (ordered by pixel (j, i) and sub-sample (is, js)) and cell_values [num_values][num_cells] (internal units; of an
        averaged map -- a TemperatureProbe's -- the weights of the cells)"""
        import numpy as np
        assert self._setup, "call setup() first"
        L = lib()
        num_cells = int(scene_head(self).grid.num_cells)
        maps = []
        for index in range(L.skh_num_probe_maps(self._h)):
            info = ProbeMapInfo()
            if L.skh_probe_map_info(self._h, index, C.byref(info)) != 0:
                raise RuntimeError(L.skh_last_error().decode())
            origins = np.empty((info.num_rays, 3), dtype=np.float64)
            directions = np.empty((info.num_rays, 3), dtype=np.float64)
            values = np.empty((info.num_values, num_cells), dtype=np.float64)
            if (L.skh_probe_map_rays(self._h, index, origins.ctypes.data_as(C.c_void_p), directions.ctypes.data_as(C.c_void_p)) != 0
                    or L.skh_probe_map_values(self._h, index, values.ctypes.data_as(C.c_void_p)) != 0):
                raise RuntimeError(L.skh_last_error().decode())
            maps.append({"file_name": info.file_name.decode(), "nx": int(info.nx), "ny": int(info.ny), "sampling": int(info.sampling),
                         "num_values": int(info.num_values), "num_rays": int(info.num_rays), "after_setup": bool(info.after_setup),
                         "averaged": L.skh_probe_map_averaged(self._h, index) == 1, "origins": origins, "directions": directions, "cell_values": values})
        return maps

    def cell_indices(self, positions):
        """SpatialGrid::cellIndex of the positions [n][3] (skh_cell_indices): the cell that holds each, in the numbering ``Engine.trace_ray``
        reports, -1 outside the grid; a position on a wall between two cells belongs to the upper one.  The CPU restatement, on one thread, of
        ``Engine.sample_cells``"""
        import numpy as np
        assert self._setup, "call setup() first"
        r = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        out = np.full(r.shape[0], -2, dtype=np.int32)
        if lib().skh_cell_indices(self._h, r.shape[0], r.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        return out

    def adaptive_mesh(self, component=0):
        """the tree and the cell densities of an AdaptiveMeshMedium component (skh_adaptive_mesh) as a dict of numpy arrays (copies):
        node_box [nodes][6], node_dims [nodes][3] (0, 0, 0: leaf), node_link [nodes] (id of child 0, or the cell index of a leaf),
        cell_density [cells]; node 0 is the root, parents come before their children, the children of a node are consecutive"""
        import numpy as np
        assert self._setup, "call setup() first"
        mesh = AdaptiveMesh()
        if lib().skh_adaptive_mesh(self._h, component, C.byref(mesh)) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        n = mesh.num_nodes
        return {"node_box": np.ctypeslib.as_array(mesh.node_box, shape=(n, 6)).copy(),
                "node_dims": np.ctypeslib.as_array(mesh.node_dims, shape=(n, 3)).copy(),
                "node_link": np.ctypeslib.as_array(mesh.node_link, shape=(n,)).copy(),
                "cell_density": np.ctypeslib.as_array(mesh.cell_density, shape=(mesh.num_cells,)).copy()}

    def imported_mass(self, component=0):
        """Snapshot::mass() of an imported medium component (skh_imported_mass): its total effective mass, or number of entities"""
        assert self._setup, "call setup() first"
        out = C.c_double(0.)
        if lib().skh_imported_mass(self._h, component, C.byref(out)) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        return float(out.value)

    def imported_densities(self, component, positions):
        """Snapshot::density of an imported medium component at the positions [n][3] (skh_imported_densities): the mass or number density as
        the file implies; on the device when ``use_device_sampler`` was called before setup(), else on the host cores"""
        import numpy as np
        assert self._setup, "call setup() first"
        r = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        out = np.empty(r.shape[0], dtype=np.float64)
        if lib().skh_imported_densities(self._h, component, r.shape[0], r.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        return out

    def dimension(self):
        """MediumSystem::dimension: 1 spherical, 2 axisymmetric, 3 neither -- the largest over the medium components (skh_dimension)"""
        n = lib().skh_dimension(self._h)
        if n < 0:
            raise RuntimeError(lib().skh_last_error().decode())
        return int(n)

    def dust_components(self):
        """the medium components that are dust, in order: the rows of ``temperature_tables`` and ``dust_temperatures`` (empty unless the
        simulation is panchromatic, stores the radiation field and has dust)"""
        assert self._setup, "call setup() first"
        out = (C.c_int32 * 16)()
        n = lib().skh_dust_components(self._h, out)
        if n < 0:
            raise RuntimeError(lib().skh_last_error().decode())
        return [int(out[i]) for i in range(n)]

    def _heating(self):
        assert self._setup, "call setup() first"
        struct = DustHeating()
        if lib().skh_dust_heating(self._h, C.byref(struct)) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        return struct

    def temperature_tables(self):
        """the tables of the energy balance per dust component (pmc_dust_heating, include/pmc.h) as a dict of numpy arrays: what
        ``Engine.dust_temperatures`` takes.  Built at the first call (a thousand Planck integrals per component)"""
        return heating_tables_from(self._heating())

    def dust_temperatures(self, rf):
        """[H + 1][num_cells]: the equilibrium temperature of every dust component in every cell, then their mass-weighted mean, from the
        table rf[m * nbins + ell] -- the CPU restatement (skh_dust_temperatures) of the engine's kernel, equal to it bit for bit"""
        import numpy as np
        struct = self._heating()
        data = np.ascontiguousarray(rf, dtype=np.float64).reshape(-1)
        assert data.size == self.radiation_field_size
        out = np.empty((struct.num_components + 1, struct.num_cells), dtype=np.float64)
        if lib().skh_dust_temperatures(self._h, data.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        return out

    def write_probes(self, outdir, integrator=None, when=None, weighted=None, temperatures=None, rf=None, sampler=None):
        """write the probe files into outdir.  integrator: an ``Engine`` (its pmc_integrate_rays, pmc_integrate_weighted_rays and
        pmc_dust_temperatures are handed to the host library as C functions: rays and tables never pass through Python; only when a
        TemperatureProbe or DustAbsorptionPerCellProbe is among the probes written is the radiation field table downloaded from it, unless rf
        is given), or a callable (origins [n][3], directions [n][3],
        cell_values [V][num_cells]) -> sums [n][V]; None serves a ski file without projected maps.  With a callable, the TemperatureProbe
        maps need `weighted`, a callable (origins, directions, cell_weights [num_cells], cell_values [V][num_cells]) -> sums [n][1 + V]
        (the raw sums of pmc_integrate_weighted_rays), and the temperatures come from `temperatures`, a callable (tables) ->
        [H + 1][num_cells], or else are computed by the host from `rf`, the table rf[m * nbins + ell].  when: "Setup" or "Run" for the
        probes with that probeAfter only, None for all.  sampler: what a ConvergenceCutsProbe takes its gridded cuts from -- an ``Engine``
        (its pmc_sample_cells is handed over as a C function; the same engine as the integrator, if that is one), or a callable
        (positions [n][3], cell_values [V][num_cells]) -> values [V][n], the cell values at ``cell_indices(positions)`` and 0 outside the grid;
        without one such a probe fails ("needs a sampler")"""
        import numpy as np
        assert self._setup, "call setup() first"
        os.makedirs(outdir, exist_ok=True)
        code = {None: -1, "Setup": 0, "Run": 1}[when]
        failure = []
        keep = []
        engine = ProbeEngine()
        num_cells = int(scene_head(self).grid.num_cells)
        if hasattr(integrator, "integrate_callback"):
            engine.integrate, engine.user = integrator.integrate_callback()
            needs_field = lib().skh_probes_need_radiation_field(self._h, code) == 1
            if needs_field:
                # (an engine without these entry points -- an older libpmc.so -- gives None: the host layer then says what the probe lacks)
                engine.integrate_weighted = getattr(integrator, "weighted_callback", lambda: (None, None))()[0]
                engine.temperatures = getattr(integrator, "temperature_callback", lambda: (None, None))()[0]
                if rf is None and integrator.radiation_field_size == self.radiation_field_size:
                    rf = integrator.download_radiation_field()

        def array(pointer, *shape):
            return np.ctypeslib.as_array(pointer, shape=shape)

        def trampoline(prototype, body):
            # a C function of `prototype` around body(the arguments after `user`): 0, or 1 with the exception kept for below
            def call(_, *arguments):
                try:
                    body(*arguments)
                    return 0
                except Exception as error:  # (an exception must not cross the C frames: reported below)
                    failure.append(error)
                    return 1

            keep.append(prototype(call))
            return C.cast(keep[-1], C.c_void_p)

        if integrator is not None and not hasattr(integrator, "integrate_callback"):
            def call(n, origins, directions, num_values, values, sums):
                result = integrator(array(origins, n, 3), array(directions, n, 3), array(values, num_values, num_cells))
                array(sums, n, num_values)[:] = np.asarray(result, dtype=np.float64).reshape(n, num_values)

            engine.integrate = trampoline(INTEGRATE_FN, call)
        if weighted is not None:
            def call_weighted(n, origins, directions, num_values, weights, values, sums):
                result = weighted(array(origins, n, 3), array(directions, n, 3), array(weights, num_cells), array(values, num_values, num_cells))
                array(sums, n, 1 + num_values)[:] = np.asarray(result, dtype=np.float64).reshape(n, 1 + num_values)

            engine.integrate_weighted = trampoline(INTEGRATE_WEIGHTED_FN, call_weighted)
        if temperatures is not None:
            def call_temperatures(tables, out):
                struct = DustHeating.from_address(tables)
                shape = (struct.num_components + 1, struct.num_cells)
                array(out, *shape)[:] = np.asarray(temperatures(heating_tables_from(struct)), dtype=np.float64).reshape(shape)

            engine.temperatures = trampoline(TEMPERATURE_FN, call_temperatures)
        if rf is not None:
            table = np.ascontiguousarray(rf, dtype=np.float64).reshape(-1)
            assert table.size == self.radiation_field_size
            keep.append(table)
            engine.rf = table.ctypes.data
        sample = None
        if hasattr(sampler, "sample_callback"):
            sample, user = sampler.sample_callback()
            address = user if isinstance(user, int) or user is None else C.cast(user, C.c_void_p).value
            if engine.user is not None and engine.user != address:
                raise ValueError("integrator and sampler must be the same engine")
            engine.user = user
        elif sampler is not None:
            def call_sample(n, positions, num_values, values, out, cells):
                r = array(positions, n, 3)
                array(out, num_values, n)[:] = np.asarray(sampler(r, array(values, num_values, num_cells)), dtype=np.float64).reshape(num_values, n)
                if cells:
                    array(cells, n)[:] = self.cell_indices(r)

            sample = trampoline(SAMPLE_FN, call_sample)
        if lib().skh_write_probes_sampled(self._h, C.byref(engine), sample, os.fsencode(outdir), code) != 0:
            if failure:
                raise failure[0]
            raise RuntimeError(lib().skh_last_error().decode())

    def save_scene(self, path):
        """the set-up scene as one file (skh_scene_save): other processes of a multi-GPU job load it with SceneFile instead of
        repeating the setup"""
        assert self._setup, "call setup() first"
        if lib().skh_scene_save(self._h, os.fsencode(path)) != 0:
            raise RuntimeError(lib().skh_last_error().decode())

    def summary(self):
        buf = C.create_string_buffer(2048)
        lib().skh_summary(self._h, buf, len(buf))
        return buf.value.decode()

    def write(self, frames, outdir):
        """calibrate a COPY of the detector arrays (numpy float64) and write the output files into outdir"""
        import numpy as np
        data = np.ascontiguousarray(frames, dtype=np.float64).copy()
        assert data.size == self.frame_size
        os.makedirs(outdir, exist_ok=True)
        if lib().skh_write(self._h, data.ctypes.data_as(C.c_void_p), os.fsencode(outdir)) != 0:
            raise RuntimeError(lib().skh_last_error().decode())
        return data


class SceneFile:
    """A scene saved by ``Simulation.save_scene``: what the engine needs (``scene``, ``seed``, ``frame_size``, ``layout``,
    ``radiation_field_size``), without the model behind it -- the process that holds the Simulation writes the output."""

    def __init__(self, path):
        L = lib()
        self.path = str(path)
        self._f = L.skh_scene_load(os.fsencode(path))
        if not self._f:
            raise RuntimeError(L.skh_last_error().decode())

    def close(self):
        if getattr(self, "_f", None):
            lib().skh_scene_file_free(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def scene(self):
        return ScenePointer(lib().skh_scene_file_scene(self._f), lib().skh_scene_file_scene_ext(self._f))

    @property
    def phase_functions(self):
        return list(SceneExt.from_address(lib().skh_scene_file_scene_ext(self._f)).phase_function)

    @property
    def source_velocities(self):
        return [v.as_dict() for v in SceneExt.from_address(lib().skh_scene_file_scene_ext(self._f)).source_velocity]

    def _number(self, what):
        return int(lib().skh_scene_file_number(self._f, what))

    seed = property(lambda self: self._number(0))
    num_packets = property(lambda self: self._number(1))
    frame_size = property(lambda self: self._number(2))
    radiation_field_size = property(lambda self: self._number(3))
    setup_draws = property(lambda self: self._number(4))

    def layout(self, instrument=0):
        out = FrameLayout()
        if lib().skh_scene_file_layout(self._f, instrument, C.byref(out)) != 0:
            raise IndexError(instrument)
        return out

