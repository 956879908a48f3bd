"""Pins what the CPU oracle (oracle/life_cycle.cpp) does with a scene's extension -- the dipole phase function of electron components, the
Doppler shift of moving sources -- and with binary trees against the UNMODIFIED reference: with the reference's own mt19937_64 stream,
one thread, the oracle reproduces the files that oracle/_ref wrote (tests/golden/make_golden_extended.py) BYTE FOR BYTE, as
tests/test_oracle_golden.py does for the scenes without an extension.  The GPU engine is then held to this oracle history by history
(tests/test_gpu_extended_oracle.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from conftest import golden, ski
from skirt9_amd.host import CounterValues, SceneExt, Simulation
from test_oracle_golden import _same_file

PMC_ERR_UNSUPPORTED = -2

# (scene, files of the fixture, the oracle without the extension must NOT reproduce them)
SCENES = [("cfg1elecg", 39, True), ("cfg2agneleceag", 25, True), ("cfg1elecnfg", 39, True), ("cfg1king", 25, True), ("cfg3king", 22, True),
          ("cfg2bindeep", 11, False), ("cfg2bing", 33, False), ("cfg2binall", 30, True)]


def _fixture_files(name):
    return sorted(f for f in os.listdir(golden("")) if f.startswith(name + "_") and "_rays" not in f
                  and (f.endswith(".fits") or f.endswith("_sed.dat") or f.endswith("_sedstats.dat")))


@pytest.mark.parametrize("name,nfiles,extended", SCENES)
def test_byte_identical_to_reference(name, nfiles, extended, tmp_path):
    """cfg1elecg: free electrons on the Cartesian grid, forced scattering, two scattering levels recorded; cfg2agneleceag: electrons next to
    dust on an octree, explicit absorption (the dipole value inside the consolidated sum over components, the component pick); cfg1elecnfg:
    electrons without forced scattering; cfg1king: a moving point source, five instruments, one observer shared, one in the observer
    frame of a redshift; cfg3king: a rotating disk (cylindrical field) and a moving point source in dust that is steep in wavelength;
    cfg2bindeep: a binary tree of 36 levels; cfg2bing: reduced cfg2bin; cfg2binall: a binary tree holding one electron component,
    panchromatic, with a rotating disk of sources and three observers.  Every FITS cube, SED and statistics table of the fixture."""
    sim = Simulation(ski(name + ".ski")).setup()
    frames, counters = O.run_primary(sim, 0, sim.num_packets, O.RNG_MT19937, ext=True)
    assert counters.histories == sim.num_packets == 20000 and counters.scatterings > sim.num_packets // 2
    sim.write(frames, str(tmp_path))
    expected = _fixture_files(name)
    assert len(expected) == nfiles
    for f in expected:
        assert os.path.exists(tmp_path / f), f
        assert _same_file(golden(f), str(tmp_path / f)), f"{f} differs from the reference output"
    if extended:
        # the files tell the extension apart: read as Henyey-Greenstein and at rest, the same scene gives other files
        plain, _ = O.run_primary(sim, 0, sim.num_packets, O.RNG_MT19937)
        other = tmp_path / "plain"
        other.mkdir()
        sim.write(plain, str(other))
        assert sum(not _same_file(golden(f), str(other / f)) for f in expected) >= 3


def _run_ext(sim, ext, n, rng_kind=O.RNG_PHILOX, seed=7, rf=False):
    """oracle_run_primary_ext with an extension of the caller's making (an address, a SceneExt, or None); returns (status, frames, rf)"""
    frames = np.zeros(sim.frame_size, dtype=np.float64)
    field = np.zeros(sim.radiation_field_size, dtype=np.float64) if rf else None
    counters = CounterValues()
    where = C.addressof(ext) if isinstance(ext, SceneExt) else ext
    rc = O.lib().oracle_run_primary_ext(int(sim.scene), where, 0, n, rng_kind, seed, sim.setup_draws if rng_kind == O.RNG_MT19937 else 0,
                                        frames.ctypes.data_as(C.c_void_p), field.ctypes.data_as(C.c_void_p) if rf else None, C.byref(counters))
    return rc, frames, field


def _copy_of_extension(sim):
    ext = SceneExt()
    C.memmove(C.addressof(ext), sim.scene.ext, C.sizeof(SceneExt))
    assert ext.struct_size == C.sizeof(SceneExt)
    return ext


@pytest.mark.parametrize("name,rng_kind,rf", [("cfg2small", O.RNG_MT19937, False), ("cfg3small", O.RNG_PHILOX, False), ("cfg1mmrf", O.RNG_PHILOX, True),
                                              ("cfg1elecg", O.RNG_PHILOX, False), ("cfg1king", O.RNG_MT19937, False)])
def test_entry_points_without_an_extension_agree(name, rng_kind, rf):
    """oracle_run_primary / oracle_run_primary_rf keep their meaning: the new entry point with ext = NULL returns the same arrays, bit for
    bit -- also for a scene that HAS an extension (no extension means Henyey-Greenstein and at rest)"""
    n = 3000
    sim = Simulation(ski(name + ".ski"), num_packets=n).setup()
    rc, frames, field = _run_ext(sim, None, n, rng_kind, seed=sim.seed if rng_kind == O.RNG_MT19937 else 7, rf=rf)
    assert rc == 0 and frames.sum() > 0
    if rf:
        old, old_field, _ = O.run_primary_rf(sim, 0, n, rng_kind, seed=7)
        assert np.array_equal(field, old_field) and field.sum() > 0
    else:
        old, _ = O.run_primary(sim, 0, n, rng_kind, seed=sim.seed if rng_kind == O.RNG_MT19937 else 7)
    assert np.array_equal(frames, old)


def test_struct_size_is_honoured():
    """members beyond struct_size do not exist (as for pmc_create_ext): an extension that ends before the phase functions is no extension,
    one that ends before the velocities has every source at rest"""
    n = 2000
    sim = Simulation(ski("cfg2binall.ski"), num_packets=n).setup()
    full = _copy_of_extension(sim)
    assert full.phase_function[0] == 1 and full.source_velocity[0].kind == 3
    plain = _run_ext(sim, None, n)[1]
    whole = _run_ext(sim, full, n)[1]
    short = _copy_of_extension(sim)
    short.struct_size = C.sizeof(C.c_int32)
    assert np.array_equal(_run_ext(sim, short, n)[1], plain)
    at_rest = _copy_of_extension(sim)
    at_rest.struct_size = SceneExt.source_velocity.offset
    dipole_only = _run_ext(sim, at_rest, n)[1]
    static = _copy_of_extension(sim)
    static.source_velocity[0].kind = 0
    assert np.array_equal(dipole_only, _run_ext(sim, static, n)[1])
    assert not np.array_equal(dipole_only, plain) and not np.array_equal(dipole_only, whole) and not np.array_equal(whole, plain)
    unset = _copy_of_extension(sim)
    unset.struct_size = 0
    assert _run_ext(sim, unset, n)[0] == -1      # PMC_ERR_INVALID, as pmc_create_ext


def test_what_the_engine_refuses_is_refused():
    """an unknown phase function kind, an unknown velocity kind, a moving source next to several medium components or a stored radiation
    field: PMC_ERR_UNSUPPORTED, as from pmc_create_ext -- never read as something else"""
    n = 100
    sim = Simulation(ski("cfg1elecg.ski"), num_packets=n).setup()
    ext = _copy_of_extension(sim)
    ext.phase_function[0] = 2
    assert _run_ext(sim, ext, n)[0] == PMC_ERR_UNSUPPORTED
    ext.phase_function[0] = -1
    assert _run_ext(sim, ext, n)[0] == PMC_ERR_UNSUPPORTED
    # (a kind in the slot of a component the scene does not have is not looked at)
    ext = _copy_of_extension(sim)
    ext.phase_function[3] = 9
    assert _run_ext(sim, ext, n)[0] == 0
    sim = Simulation(ski("cfg1king.ski"), num_packets=n).setup()
    for kind in (4, -1):
        ext = _copy_of_extension(sim)
        ext.source_velocity[0].kind = kind
        assert _run_ext(sim, ext, n)[0] == PMC_ERR_UNSUPPORTED
    moving = _copy_of_extension(sim).source_velocity[0]
    assert moving.kind == 1
    # panchromatic scenes with two medium components / with a stored radiation field, handed a moving source
    for name, rf in (("cfg3mm", False), ("cfg3rf", True)):
        sim = Simulation(ski(name + ".ski"), num_packets=n).setup()
        ext = _copy_of_extension(sim)
        assert _run_ext(sim, ext, n, rf=rf)[0] == 0
        ext.source_velocity[0] = moving
        assert _run_ext(sim, ext, n, rf=rf)[0] == PMC_ERR_UNSUPPORTED
    # (SpecialtySource.cpp:34-44: no velocity in an oligochromatic simulation -- such a source is at rest, not refused)
    sim = Simulation(ski("cfg1mmrf.ski"), num_packets=n).setup()
    ext = _copy_of_extension(sim)
    ext.source_velocity[0] = moving
    rc, frames, _ = _run_ext(sim, ext, n, rf=True)
    assert rc == 0 and np.array_equal(frames, _run_ext(sim, None, n, rf=True)[1])


def test_velocity_fields_follow_the_closed_forms():
    """the oracle's source velocity through what it does to the light: a face-on observer of cfg2binall sees no shift from a rotation about
    the z-axis, an edge-on observer sees the line spread over more than three of its wavelength bins; at rest both see it in at most two"""
    n = 4000
    sim = Simulation(ski("cfg2binall.ski"), num_packets=n).setup()
    moving, _ = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=3, ext=True)
    rest, _ = O.run_primary(sim, 0, n, O.RNG_PHILOX, seed=3)
    edge, face = sim.layout(0), sim.layout(2)
    row = lambda frames, lay: frames[lay.sed_offset:lay.sed_offset + lay.num_lambda]      # the transparent component
    assert np.count_nonzero(row(rest, edge)) <= 2 and np.count_nonzero(row(rest, face)) <= 2
    assert np.count_nonzero(row(moving, edge)) > 3
    assert np.array_equal(row(moving, face) > 0, row(rest, face) > 0)
